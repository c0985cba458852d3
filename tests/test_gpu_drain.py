"""Output pipeline on the GPU: the int16 plane packing and the fp32 staging kernel against the numpy restatement of
tests/test_drain_cpu.py, data.HostDrain (ordering, staging races, back-pressure, errors) and rollout.rollout(drain=...)."""
import threading
import time

import numpy as np
import pytest
import torch

import cases
import synth
from test_drain_cpu import FILL, contract_violations, endpoints_ok, pack_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    P._lib.load()
    return P


def gpu_pack(P, x, mul=None, add=None, levels=0):
    """x (planes, H, W) fp32 on the GPU -> (q, scale_offset, nonfinite) as numpy, through the C ABI on the current stream."""
    lib = P._lib.load()
    planes, elems = x.shape[0], x.shape[1] * x.shape[2]
    ws_bytes = lib.pangu_pack_i16_ws_bytes(planes, elems)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 4 + 16,), float("nan"), device="cuda")        # (no zero-initialised memory is needed)
    q = torch.full((planes * elems + 8,), 12345, dtype=torch.int16, device="cuda")      # 8 guard values behind the output
    so = torch.full((planes, 2), float("nan"), device="cuda")
    nf = torch.full((planes,), -1, dtype=torch.int32, device="cuda")
    rc = lib.pangu_pack_planes_i16(torch.cuda.current_stream().cuda_stream, x.data_ptr(), mul.data_ptr() if mul is not None else None,
                                   add.data_ptr() if add is not None else None, q.data_ptr(), so.data_ptr(), nf.data_ptr(),
                                   ws.data_ptr(), ws_bytes, planes, elems, levels)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (q[planes * elems:] == 12345).all() and torch.isnan(ws[ws_bytes // 4:]).all()
    return q[:planes * elems].view(planes, elems).cpu().numpy(), so.cpu().numpy(), nf.cpu().numpy()


def field(shape, seed, normalised=False):
    """Planes of N(0,1) values, generated on the GPU: scaled and shifted per plane (ranges from 1e-3 to 1e3, the mean up to 10 x
    the spread), or left normalised for `affine` to de-normalise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    planes = shape[0]
    x = torch.randn(shape, generator=g, device="cuda")
    if normalised:
        return x
    amp = torch.logspace(-3, 3, planes, device="cuda").view(-1, 1, 1)
    return (x * amp + 10 * amp * torch.arange(planes, device="cuda").view(-1, 1, 1).float().cos()).contiguous()


def affine(planes, seed):
    """(std, mean) per plane as de-normalisation has them: std from 1e-3 to 1e3, |mean| up to 60 std (geopotential is 2e5 +- 5e3,
    surface pressure 101325 +- 1500).  The half-ulp rounding of a plane's offset then stays far below half a count of its scale,
    which is what lets the extremes land on +-32767 exactly."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    std = torch.logspace(-3, 3, planes, device="cuda")[torch.randperm(planes, generator=g, device="cuda")]
    return std.contiguous(), (std * (torch.rand(planes, generator=g, device="cuda") * 120 - 60)).contiguous()


def check_against_reference(P, x, mul=None, add=None, levels=0):
    q, so, nf = gpu_pack(P, x, mul, add, levels)
    planes = x.shape[0]
    rq, rso, rnf, v = pack_reference(x.reshape(planes, -1).cpu().numpy(), None if mul is None else mul.cpu().numpy(),
                                     None if add is None else add.cpu().numpy(), levels)
    assert np.array_equal(so.view(np.uint32), rso.view(np.uint32))            # min / max are order-independent: bit for bit
    assert np.array_equal(nf, rnf)
    bad, worst = contract_violations(q, so, v)
    dq = np.abs(q.astype(np.int32) - rq.astype(np.int32)).max()
    print(f"shape {tuple(x.shape)} affine={mul is not None} levels={levels}: worst |error| / bound = {worst:.3f}, max |dq| = {dq}")
    assert bad == 0
    assert dq <= 1
    assert endpoints_ok(q, v)


# one partial slab; 156 values per plane (a multiple of 4, not of 8); odd plane size (plane 1 starts 2-B aligned in the int16
# output and 4-B aligned in the input: scalar head and tail); many slabs per plane
SHAPES = [(3, 5, 8), (7, 13, 12), (2, 3, 5), (2, 181, 360)]


@pytest.mark.parametrize("with_affine", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_pack_kernel_vs_reference(P, shape, with_affine):
    x = field(shape, 11, normalised=with_affine)
    mul, add = affine(shape[0], 12) if with_affine else (None, None)
    check_against_reference(P, x, mul, add)


def test_pack_kernel_level_reversal(P):
    x = field((2 * 13, 9, 16), 13, normalised=True)
    mul, add = affine(26, 14)
    check_against_reference(P, x, mul, add, levels=13)


def test_pack_kernel_full_grid(P):
    """69 planes of 721 x 1440: the real grid (64 slabs per plane, 286 MB of input)."""
    x = field((69, 721, 1440), 15, normalised=True)
    mul, add = affine(69, 16)
    check_against_reference(P, x, mul, add)


def test_pack_kernel_edge_planes(P):
    x = field((4, 9, 21), 17)                       # 189 values per plane: odd, so the planes differ in alignment
    x[0] = 271.5                                    # constant
    x[1, 2, 3] = float("nan")
    x[1, 7, 20] = float("inf")
    x[2] = float("nan")
    x[2, 1] = float("-inf")                         # no finite value at all
    q, so, nf = gpu_pack(P, x)
    rq, rso, rnf, v = pack_reference(x.reshape(4, -1).cpu().numpy())
    assert np.array_equal(so.view(np.uint32), rso.view(np.uint32)) and np.array_equal(nf, rnf)
    assert (q[0] == 0).all() and tuple(so[0]) == (1.0, 271.5) and nf[0] == 0
    assert q[0].astype(np.float32)[0] * so[0, 0] + so[0, 1] == 271.5              # unpacks exactly
    assert nf[1] == 2 and q[1][2 * 21 + 3] == FILL and q[1][7 * 21 + 20] == FILL and (q[1] == FILL).sum() == 2
    fin = np.isfinite(v[1])
    assert so[1, 1] == np.float32((v[1][fin].max() + v[1][fin].min()) / np.float32(2))       # min / max ignore them
    assert nf[2] == 189 and (q[2] == FILL).all() and np.isfinite(so[2]).all()
    assert contract_violations(q, so, v)[0] == 0 and endpoints_ok(q, v)
    assert np.abs(q.astype(np.int32) - rq.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("shape,levels", [((3, 5, 8), 0), ((2, 3, 5), 0), ((26, 9, 16), 13), ((26, 9, 15), 13), ((2, 181, 360), 2)])
@pytest.mark.parametrize("with_affine", [False, True])
def test_stage_kernel_equals_torch(P, shape, levels, with_affine):
    lib = P._lib.load()
    x = field(shape, 21)
    planes, elems = shape[0], shape[1] * shape[2]
    mul, add = affine(planes, 22) if with_affine else (None, None)
    out = torch.full((planes * elems + 4,), float("nan"), device="cuda")
    rc = lib.pangu_stage_planes_f32(torch.cuda.current_stream().cuda_stream, x.data_ptr(), mul.data_ptr() if with_affine else None,
                                    add.data_ptr() if with_affine else None, out.data_ptr(), planes, elems, levels)
    assert rc == 0, rc
    want = x * mul.view(-1, 1, 1) + add.view(-1, 1, 1) if with_affine else x
    if levels:
        want = want.view(planes // levels, levels, *shape[1:]).flip(1).reshape(shape)
    assert torch.equal(out[:planes * elems].view(shape), want) and torch.isnan(out[planes * elems:]).all()


PAIR = [(2, 13, 9, 16), (4, 9, 16)]


def pair(k):
    g = torch.Generator(device="cuda").manual_seed(100 + k)
    return [torch.randn(s, generator=g, device="cuda") * (k + 1) + 3 * k for s in PAIR]


def copy_item(item, mode):
    if mode == "int16":
        return item.tag, [(f.packed.copy(), f.scale_offset.copy(), f.nonfinite.copy()) for f in item.fields]
    return item.tag, [f.values.copy() for f in item.fields]


def check_item(got, original, mode):
    for f, t in zip(got, original):
        if mode == "int16":
            rq, rso, rnf, _ = pack_reference(t.reshape(-1, 9 * 16))
            q, so, nf = f
            assert q.shape == t.shape and so.shape == rso.shape and nf.shape == rnf.shape
            assert np.array_equal(so, rso) and np.array_equal(nf, rnf)
            assert np.abs(q.reshape(rq.shape).astype(np.int32) - rq.astype(np.int32)).max() <= 1
        else:
            assert f.shape == t.shape and np.array_equal(f, t)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["int16", "float32"])
def test_host_drain_order_and_staging(P, mode):
    """Six pairs through a ring of three slots, the source poisoned right after each submit: every item arrives, in order, and
    matches the ORIGINAL values (a staging race or a slot reused too early would show NaN or another item's data)."""
    got, originals = [], []
    with P.data.HostDrain("cuda", mode=mode, depth=2, sink=lambda item: got.append(copy_item(item, mode))) as drain:
        for k in range(6):
            ts = pair(k)
            originals.append([t.cpu().numpy() for t in ts])
            drain.submit(ts, tag=k)
            for t in ts:
                t.fill_(float("nan"))
    assert [tag for tag, _ in got] == list(range(6))
    for (_, fields), orig in zip(got, originals):
        check_item(fields, orig, mode)
    st = drain.stats
    per_item = sum(int(np.prod(s)) for s in PAIR) * (2 if mode == "int16" else 4) + (12 * (26 + 4) if mode == "int16" else 0)
    assert st["items"] == 6 and st["bytes"] == 6 * per_item and len(st["d2h_events"]) == 6
    assert drain.summary()["d2h_GBps"] > 0


@pytest.mark.timeout(120)
def test_host_drain_back_pressure(P):
    got = []

    def slow(item):
        time.sleep(0.05)
        got.append(copy_item(item, "int16"))

    originals = []
    drain = P.data.HostDrain("cuda", mode="int16", depth=2, sink=slow)
    for k in range(6):
        ts = pair(k)
        originals.append([t.cpu().numpy() for t in ts])
        drain.submit(ts, tag=k)
    drain.close()
    assert [tag for tag, _ in got] == list(range(6))
    for (_, fields), orig in zip(got, originals):
        check_item(fields, orig, "int16")
    assert drain.stats["producer_wait_s"] > 0.04          # submits 4-6 each waited for the sleeping sink to release a slot


@pytest.mark.timeout(120)
def test_host_drain_sink_error_reaches_close(P):
    def broken(item):
        raise KeyError("disk full")

    drain = P.data.HostDrain("cuda", mode="int16", depth=2, sink=broken)
    drain.submit(pair(0), tag=0)
    with pytest.raises(KeyError, match="disk full"):
        drain.close()
    assert not any(t.name == "pangu-drain" and t.is_alive() for t in threading.enumerate())


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["int16", "float32"])
def test_host_drain_get_without_sink(P, mode):
    drain = P.data.HostDrain("cuda", mode=mode, depth=2, copy_threads=2)
    originals = []
    for k in range(2):
        ts = pair(k)
        originals.append([t.cpu().numpy() for t in ts])
        drain.submit(ts, tag=k)
        for t in ts:
            t.fill_(float("nan"))
    first = drain.get()
    assert first.tag == 0
    check_item(copy_item(first, mode)[1], originals[0], mode)
    # to_float32 is the C-ABI unpack: the numpy expression, bit for bit
    f0 = first.fields[0]
    want = (f0.packed.reshape(26, -1).astype(np.float32) * f0.scale_offset[:, :1] + f0.scale_offset[:, 1:]).reshape(PAIR[0]) \
        if mode == "int16" else f0.values
    assert np.array_equal(first.to_float32()[0], want)
    second = drain.get()                                    # releases `first`
    assert second.tag == 1 and first.fields == []
    check_item(copy_item(second, mode)[1], originals[1], mode)
    assert drain.get() is None
    drain.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["int16", "float32"])
def test_host_drain_denormalises_and_flips(P, mode):
    """stats_last + flip_levels: a normalised (1,5,13,H,W) / (1,4,H,W) pair arrives de-normalised (rollout.norm_back's arithmetic,
    bit for bit in float32 mode) with the level axis of the upper-air tensor reversed."""
    g = torch.Generator(device="cuda").manual_seed(7)
    up, sf = torch.randn((1, 5, 13, 9, 16), generator=g, device="cuda"), torch.randn((1, 4, 9, 16), generator=g, device="cuda")
    u_std, u_mean = (t.view(1, 5, 13, 1, 1) for t in affine(65, 31))
    s_std, s_mean = (t.view(1, 4, 1, 1) for t in affine(4, 32))
    sl = (s_mean, s_std, u_mean, u_std)
    want_up, want_sf = P.rollout.norm_back(up, sf, sl)
    want_up = want_up.flip(2)
    drain = P.data.HostDrain("cuda", mode=mode, depth=1, stats_last=sl, flip_levels=True)
    drain.submit([up, sf], tag="t0")
    item = drain.get()
    assert item.tag == "t0"
    if mode == "float32":
        assert np.array_equal(item.fields[0].values, want_up.cpu().numpy()) and np.array_equal(item.fields[1].values, want_sf.cpu().numpy())
    else:
        for f, x, std, mean, levels, want in ((item.fields[0], up, u_std, u_mean, 13, want_up), (item.fields[1], sf, s_std, s_mean, 0, want_sf)):
            planes = f.scale_offset.shape[0]
            rq, rso, rnf, v = pack_reference(x.reshape(planes, -1).cpu().numpy(), std.reshape(-1).cpu().numpy(),
                                             mean.reshape(-1).cpu().numpy(), levels)
            assert np.array_equal(v, want.reshape(planes, -1).cpu().numpy())              # the oracle's own value is norm_back + flip
            assert f.packed.shape == tuple(x.shape) and np.array_equal(f.scale_offset, rso) and np.array_equal(f.nonfinite, rnf)
            q = f.packed.reshape(planes, -1)
            assert np.abs(q.astype(np.int32) - rq.astype(np.int32)).max() <= 1
            assert contract_violations(q, f.scale_offset, v)[0] == 0 and endpoints_ok(q, v)
    drain.close()


@pytest.fixture(scope="module")
def setup(P):
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return m, cases.model_inputs("cuda")


def _stats_last(stats):
    s_mean, s_std, u_mean, u_std = stats
    return (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("graph", [True, False])
def test_rollout_drains_every_step(P, setup, graph):
    """fp32, 2 steps, full model: the final state is untouched by drain=, and every drained lead time meets the error contract
    against norm_back of the corresponding keep=True output."""
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    up0, sf0, hist = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, keep=True)
    got = []
    with P.data.HostDrain("cuda", mode="int16", depth=2, sink=lambda item: got.append(copy_item(item, "int16"))) as drain:
        up1, sf1 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, drain=drain)
    assert torch.equal(up0, up1) and torch.equal(sf0, sf1)
    assert [tag for tag, _ in got] == [0, 1]
    for (_, fields), (out, out_s) in zip(got, hist):
        for (q, so, nf), want in zip(fields, P.rollout.norm_back(out, out_s, sl)):
            assert q.shape == tuple(want.shape) and nf.sum() == 0
            planes = so.shape[0]
            # the contract in fp64 on the GPU (71.6 M values): |q * scale + offset - v| against the per-plane bound
            v = want.reshape(planes, -1).double()
            s, o = (torch.from_numpy(so[:, k].astype(np.float64)).cuda().view(-1, 1) for k in (0, 1))
            err = (torch.from_numpy(q.reshape(planes, -1)).cuda().double() * s + o - v).abs()
            bound = 0.5 * s * (1 + 2.0 ** -10) + 4 * 2.0 ** -24 * torch.maximum(v.min(1, keepdim=True).values.abs(),
                                                                               v.max(1, keepdim=True).values.abs())
            worst = (err / bound).max().item()
            print(f"graph={graph} planes={planes}: worst |error| / bound = {worst:.3f}")
            assert bool((err <= bound).all())
