"""Layer modules of the Pangu-Weather network, MI355X-native.

Mirror of the reference's module tree (models/layers.py): same class names, constructor arguments,
sub-module names and parameter shapes, so `state_dict()` keys/shapes match the 223-row keys_all.csv and
`named_modules()` introspection (LoRA targets, torch_summarize) keeps working.  The arithmetic is NOT the
reference's op chain: every forward calls hand-written gfx950 kernels through the C ABI (`ops.py`), with
all view/pad/roll/permute/crop steps folded into kernel address arithmetic.  nn.Linear / nn.Conv1d /
nn.LayerNorm sub-modules are parameter containers only.
"""
import math
import weakref
from collections import OrderedDict

import torch
from torch import nn

from . import fused

WINDOW = (2, 6, 12)


def _trunc_normal_(t, std):
    return nn.init.trunc_normal_(t, std=std)      # stands in for timm's trunc_normal_ (reference layers.py:9)


class DropPath(nn.Module):
    """Stochastic depth (timm semantics, reference layers.py:140): in training each residual branch of a
    sample is dropped with prob p, else scaled 1/(1-p).  Only the per-sample factor is drawn here; it is
    applied inside the fused LayerNorm-residual kernel (and a dropped branch is not computed at all)."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)
        self.n_dropped = 0           # branches dropped so far (diagnostic)
        self.n_dropped_branch = [0, 0]      # ... split by branch: [attention (layers.py:250), MLP (:251)]; bench.py prices the
                                            # work a training step really executed with these
        self._calls = 0

    def sample_scale(self, training):
        """The per-sample factor of the next residual branch; a block draws twice per sample, attention branch first."""
        which = self._calls & 1
        self._calls += 1
        if not training or self.drop_prob == 0.0:
            return 1.0
        keep = 1.0 - self.drop_prob
        if torch.rand(()).item() < keep:
            return 1.0 / keep
        self.n_dropped += 1
        self.n_dropped_branch[which] += 1
        return 0.0

    def extra_repr(self):
        return f"drop_prob={self.drop_prob:.3f}"


def _lowbias32(x):
    """csrc/common.h lowbias32 on an int64 tensor holding uint32 values."""
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & m
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & m
    return x ^ (x >> 16)


def lora_dropout_threshold(p):
    """T of the keep mask: clamp(floor(p * 2^32 + 0.5), 1, 2^32 - 1), computed from the double `p` (as csrc/common.h does)."""
    return min(max(int(math.floor(float(p) * 4294967296.0 + 0.5)), 1), 0xFFFFFFFF)


def lora_dropout_keep(seed, M, K, p, device=None):
    """The keep mask of the adapter dropout on an (M, K) adapter input, a pure function of (seed, row, column): the host
    restatement of what the kernels recompute (csrc/common.h, LoraDrop) -> bool (M, K), True where the entry is kept:
        keep(seed, i, k) = lowbias32(lowbias32(lowbias32(seed) ^ i) ^ k) >= T,  T = lora_dropout_threshold(p)
    Integer torch ops (usable on the CPU); seed is a uint32."""
    seed = int(seed)
    if not 0 <= seed <= 0xFFFFFFFF:
        raise ValueError(f"lora_dropout_keep: seed {seed} is not a uint32")
    hs = _lowbias32(torch.tensor(seed, dtype=torch.int64, device=device))
    hrow = _lowbias32(hs ^ torch.arange(M, dtype=torch.int64, device=device))
    return _lowbias32(hrow[:, None] ^ torch.arange(K, dtype=torch.int64, device=device)[None, :]) >= lora_dropout_threshold(p)


def draw_lora_dropout_seed():
    """One uint32 from torch's default CPU generator (the generator DropPath.sample_scale draws from): `torch.manual_seed`
    reproduces the masks, and the checkpointed training steps, which restore the host RNG state, recompute with the same ones."""
    return int(torch.randint(0, 1 << 32, (), dtype=torch.int64))


class LoraLinear(nn.Linear):
    """An nn.Linear with a LoRA adapter (peft's `lora.Linear`, reference finetune/lora_tune.py:124-135): y = x W_eff^T + b with
    W_eff = W + scaling * lora_B @ lora_A, scaling = alpha / r.  `weight` / `bias` are the frozen base parameters under their own
    names (the base state_dict keys do not change); `lora_A` (r, in) starts kaiming-uniform, `lora_B` (out, r) at zero, as peft
    initialises them, so a fresh adapter computes exactly what the base layer computes.

    The kernels never see A and B in the forward: they run on W_eff (`effective_weight()`), a derived tensor made by
    `pangu_lora_merge_f32` and re-made only when the stamp (ops.param_stamp) of W, A or B changes -- like the bf16 weight
    shadows, it is never pickled and is dropped by `.to()` / `invalidate_shadows`.  The adapter gradients come from
    `pangu_lora_wgrad_f32` (`pangu_lora_wgrad_bf16` on the bf16 training path) in the backward of the layer functions (autograd.py).

    `lora_dropout` (peft's name; default 0): in train() mode the adapter path reads drop(x) = keep * x / (1 - p) instead of x,
    y = x W^T + b + s drop(x) A^T B^T.  The mask is lora_dropout_keep of a seed drawn per call (`last_dropout_seed` keeps the
    latest); the layer functions apply it as additive corrections around the W_eff launches (csrc/lora_dropout_f32.hip, and
    csrc/lora_dropout_bf16.hip on the bf16 training path)."""

    def __init__(self, in_features, out_features, bias=True, r=16, alpha=16, device=None, dtype=None, lora_dropout=0.0):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self._init_lora(r, alpha, lora_dropout)

    def _init_lora(self, r, alpha, lora_dropout=0.0):
        self.r, self.lora_alpha = int(r), alpha
        self.scaling = alpha / r
        self.lora_dropout = float(lora_dropout)
        if not 0.0 <= self.lora_dropout < 1.0:
            raise ValueError(f"LoraLinear: lora_dropout={lora_dropout} is not in [0, 1)")
        self.last_dropout_seed = None
        w = self.weight
        self.lora_A = nn.Parameter(torch.empty((self.r, self.in_features), device=w.device, dtype=w.dtype))
        self.lora_B = nn.Parameter(torch.zeros((self.out_features, self.r), device=w.device, dtype=w.dtype))
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
        self._w_eff = None
        self._w_eff_stamp = None

    @classmethod
    def from_linear(cls, lin, r, alpha, lora_dropout=0.0):
        """Adapt `lin` in place of it: the new module holds the SAME weight / bias Parameter objects."""
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.in_features, m.out_features = lin.in_features, lin.out_features
        m.weight = lin.weight
        m.bias = lin.bias
        m._init_lora(r, alpha, lora_dropout)
        return m

    def to_linear(self, weight=None):
        """A plain nn.Linear holding this module's base Parameters (merge_lora folds W_eff into `weight` first)."""
        lin = nn.Linear.__new__(nn.Linear)
        nn.Module.__init__(lin)
        lin.in_features, lin.out_features = self.in_features, self.out_features
        lin.weight = self.weight
        lin.bias = self.bias
        return lin

    def _stamp(self):
        from . import ops
        return (ops.param_stamp(self.weight), ops.param_stamp(self.lora_A), ops.param_stamp(self.lora_B), self.scaling)

    def effective_weight(self):
        """W_eff = W + scaling * B @ A (no autograd edge; fp32): the HIP kernel's result on a HIP device (fresh tensor per refresh,
        so a backward still holding the previous one is unaffected), plain torch on the CPU."""
        stamp = self._stamp()
        if self._w_eff is not None and self._w_eff_stamp == stamp:
            return self._w_eff
        with torch.no_grad():
            if self.weight.is_cuda:
                from . import ops
                with torch.cuda.device(self.weight.device):
                    w = ops.lora_merge(self.weight.detach(), self.lora_A.detach(), self.lora_B.detach(), self.scaling)
            else:
                w = self.weight.detach() + self.scaling * (self.lora_B.detach() @ self.lora_A.detach())
        # (the bf16 weight shadows key their images of W_eff by this module, not by the per-refresh tensor: WeightShadow._lora_owner)
        w._lora_owner = weakref.ref(self)
        self._w_eff, self._w_eff_stamp = w, stamp
        return w

    def drop_derived(self):
        self._w_eff = None
        self._w_eff_stamp = None

    def dropout_active(self):
        return self.training and getattr(self, "lora_dropout", 0.0) > 0.0

    def next_dropout_seed(self):
        """Draw (and remember) the seed of this projection's next mask."""
        self.last_dropout_seed = draw_lora_dropout_seed()
        return self.last_dropout_seed

    def forward(self, x):
        """The module on its own, plain torch (peft's arithmetic; usable on the CPU).  In train() mode with lora_dropout > 0 the
        adapter path reads drop(x), with the kernels' mask on the rows of x flattened to (M, in_features)."""
        xa = x
        if self.dropout_active():
            p = self.lora_dropout
            keep = lora_dropout_keep(self.next_dropout_seed(), x.numel() // x.shape[-1], x.shape[-1], p, device=x.device)
            xa = x * (keep.reshape(x.shape).to(x.dtype) / (1.0 - p))
        return nn.functional.linear(x, self.weight, self.bias) + self.scaling * nn.functional.linear(
            nn.functional.linear(xa, self.lora_A), self.lora_B)

    def _apply(self, fn, *args, **kwargs):
        self.drop_derived()
        return super()._apply(fn, *args, **kwargs)

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_w_eff"] = None
        state["_w_eff_stamp"] = None
        return state

    def extra_repr(self):
        return super().extra_repr() + f", r={self.r}, alpha={self.lora_alpha}, lora_dropout={getattr(self, 'lora_dropout', 0.0)}"


def eff_weight(lin):
    """THE accessor of every kernel call site for a projection's weight: `lin.weight` of a plain nn.Linear (the same tensor as
    before adapters existed), W_eff of a LoraLinear."""
    if type(lin) is LoraLinear:
        return lin.effective_weight()
    return lin.weight


def _lora_scaling(l):
    """A projection's entry in `lora`: its scaling, or (scaling, p, seed) while its adapter dropout is active (train() mode and
    lora_dropout > 0) -- the seed of this call's mask is drawn here."""
    if l.dropout_active():
        return (l.scaling, l.lora_dropout, l.next_dropout_seed())
    return l.scaling


def dropout_active(*modules):
    """Does any LoraLinear under `modules` apply adapter dropout in its next forward?"""
    return any(type(l) is LoraLinear and l.dropout_active() for m in modules for l in m.modules())


def lora_args(*lins):
    """The trailing `lora, *ab` arguments of a layer Function (autograd.py) for its projections `lins`: the tuple of scalings, then
    lora_A, lora_B of each projection (None in every place of a plain nn.Linear); nothing when no projection is adapted.  A
    projection whose adapter dropout is active carries (scaling, p, seed) in place of its scaling; its seed is one draw from
    torch's default CPU generator per call, in the order of `lins`."""
    ad = [(_lora_scaling(l), l.lora_A, l.lora_B) if type(l) is LoraLinear else (None, None, None) for l in lins]
    if all(s is None for s, _, _ in ad):
        return ()
    return (tuple(s for s, _, _ in ad),) + tuple(t for _, A, B in ad for t in (A, B))


_ALLOWED_MODULE_TYPES = set()      # filled on first use (assert_plain_tree)


def assert_plain_tree(root, what):
    """The kernels read the parameters of the nn.Linear / nn.Conv1d / nn.LayerNorm children directly and never call their
    `forward` (nor, on the bf16 path, the forward of ANY sub-module of the model): a wrapper that replaces such a child (LoRA /
    peft `lora.Linear`, parametrizations, quantisation stubs -- reference finetune/lora_tune.py:124-135 wraps `linear1`) or a
    forward (pre-)hook on a sub-module would be ignored silently and e.g. train nothing.  Refuse instead: every sub-module of
    `root` must be one of this file's classes or the plain torch.nn class, without forward hooks (hooks on `root` itself run)."""
    allowed = _ALLOWED_MODULE_TYPES
    if not allowed:
        allowed.update({nn.Linear, LoraLinear, nn.Conv1d, nn.LayerNorm, nn.GELU, nn.Dropout, nn.Identity, nn.Sequential, DropPath,
                        PatchEmbedding_pretrain, Mlp, EarthAttention3D, EarthSpecificBlock, EarthSpecificLayer, DownSample, UpSample,
                        PatchRecovery_pretrain})
    for m in root.modules():
        if m is not root and (m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks
                              or type(m) not in allowed):
            break
    else:
        return
    name = next(n for n, q in root.named_modules() if q is m)
    if type(m) in allowed:
        raise RuntimeError(f"{what} (MI355X build): sub-module '{name}' carries forward hooks or backward hooks, but its forward is "
                           "never called (the HIP kernels read the parameters directly): the hook would be ignored")
    raise RuntimeError(f"{what} (MI355X build): sub-module '{name}' is {type(m).__module__}.{type(m).__name__}, not the plain "
                       "module the kernels read their parameters from; a wrapper's own arithmetic (LoRA adapters, "
                       "parametrizations) would be bypassed and e.g. train nothing; for LoRA use the native adapters, "
                       "PanguModel.enable_lora()")


class PatchEmbedding_pretrain(nn.Module):
    """reference layers.py:12-93."""

    # frozen fp32 inference: its projections on the exact-split bf16-MFMA kernel (PanguModel.use_split_projections sets it)
    split_projections = True

    def __init__(self, patch_size, dim):
        super().__init__()
        self.conv = nn.Conv1d(in_channels=192, out_channels=dim, kernel_size=1, stride=1)
        self.conv_surface = nn.Conv1d(in_channels=112, out_channels=dim, kernel_size=1, stride=1)
        self.window_size = WINDOW

    def forward(self, input, input_surface, statistics, maps, const_h, levels_reversed=False):
        return fused.patch_embed(self, input, input_surface, statistics, maps, const_h, levels_reversed)


class Mlp(nn.Module):
    """reference layers.py:255-270 (dropout p=0 is the identity and is not materialised)."""

    def __init__(self, dim, dropout_rate):
        super().__init__()
        self.linear1 = nn.Linear(dim, dim * 4)
        self.linear2 = nn.Linear(dim * 4, dim)
        self.activation = nn.GELU()
        self.drop = nn.Dropout(dropout_rate)

    def forward(self, x):
        assert_plain_tree(self, "Mlp")
        if self.drop.p > 0.0 and self.training:
            raise RuntimeError("Mlp (MI355X build): dropout_rate > 0 in train() mode is not implemented by the kernels (the "
                               "reference's model builds every Mlp with rate 0, layers.py:143)")
        shp = x.shape
        return fused.mlp(self, x.reshape(-1, shp[-1])).reshape(shp)


class EarthAttention3D(nn.Module):
    """reference layers.py:272-421.  Inside a block the arithmetic is the fused window-attention kernel (the block never calls
    this module's forward); `forward(x_window, mask)` keeps the module usable on its own."""

    def __init__(self, dim, heads, dropout_rate, window_size, device=None):
        super().__init__()
        self.device = device
        self.linear1 = nn.Linear(dim, dim * 3, bias=True)
        self.linear2 = nn.Linear(dim, dim)
        self.dropout_rate = float(dropout_rate)                # reference layers.py:284 (nn.Dropout; the model passes 0)
        self.head_number = heads
        self.dim = dim
        self.scale = (dim // heads) ** -0.5
        self.window_size = window_size
        input_shape = {192: (8, 186), 384: (8, 96)}[dim]                       # reference layers.py:298-301
        self.type_of_windows = (input_shape[0] // window_size[0]) * (input_shape[1] // window_size[1])
        wtok = window_size[0] * window_size[1] * window_size[2]
        self.earth_specific_bias = nn.Parameter(torch.zeros(1, self.type_of_windows, heads, wtok, wtok, device=device))
        _trunc_normal_(self.earth_specific_bias, std=0.02)
        self._construct_index()

    def forward(self, x, mask):
        """reference layers.py:360-421, the module's own calling convention: x (nLon, types, 144, C) ALREADY partitioned into
        windows (as EarthSpecificBlock.forward :216-221 hands it over), mask None or (nLon, types, 144, 144) (gen_mask, :153-181)
        -> (nLon, types, 144, C).  EarthSpecificBlock does not come through here -- its kernels fold the partition into their
        addressing -- this is for callers that use the module on its own: linear1 and linear2 on the GEMM kernel, the core on
        `pangu_attn_windows_fwd` / `_bwd` (explicit mask tensor, every slot an ordinary token), differentiable like the
        reference's module (autograd.AttentionWindowsFn)."""
        from . import ops
        from .autograd import AttentionWindowsFn
        assert_plain_tree(self, "EarthAttention3D")
        if getattr(self, "dropout_rate", 0.0) > 0.0 and self.training:
            raise RuntimeError("EarthAttention3D (MI355X build): dropout_rate > 0 in train() mode is not implemented by the kernels "
                               "(the reference's model builds every attention with rate 0, layers.py:144)")
        if x.dim() != 4 or x.shape[1] != self.type_of_windows or x.shape[2] != 144 or x.shape[3] != self.dim:
            raise RuntimeError(f"EarthAttention3D: expected (nLon, {self.type_of_windows}, 144, {self.dim}) windows, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError(f"EarthAttention3D (MI355X build) needs its input on a HIP device (got {x.device}); there is no CPU fallback")
        n_lon = x.shape[0]
        xw = x.to(torch.float32).contiguous().view(-1, self.dim)
        m = None if mask is None else mask.detach().to(device=x.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(x.device):
            if (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))) or (
                    self.training and dropout_active(self)):
                y = AttentionWindowsFn.apply(xw, eff_weight(self.linear1), self.linear1.bias, eff_weight(self.linear2),
                                             self.linear2.bias, self.earth_specific_bias, m,
                                             (n_lon, self.type_of_windows, self.head_number), *lora_args(self.linear1, self.linear2))
            else:
                qkv = ops.linear(xw, eff_weight(self.linear1), self.linear1.bias)
                o = ops.attention_windows(qkv, self.earth_specific_bias[0], m, n_lon, self.type_of_windows, self.head_number)
                y = ops.linear(o, eff_weight(self.linear2), self.linear2.bias)
        return y.view(x.shape)

    def _construct_index(self):
        """reference layers.py:319-357: `self.position_index`, int64 (20736,) in [0, 3312) -- a plain attribute there too
        (not a buffer, not in state_dict); the reference builds it and never reads it (the gather is commented out,
        :384-391).  Here it is the closed form of weights.position_index (bit-exact against the reference's loops,
        tests/test_weights.py) and what weights.expand_bias / compact_bias index with."""
        from . import weights
        self.position_index = weights.position_index()


class EarthSpecificBlock(nn.Module):
    """reference layers.py:127-253."""

    # frozen fp32 inference: qkv and MLP-up on the exact-split bf16-MFMA kernel (PanguModel.use_split_projections sets it per block)
    split_projections = True

    def __init__(self, dim, drop_path_ratio, heads, device=None):
        super().__init__()
        self.device = device
        self.window_size = WINDOW
        self.drop_path = DropPath(drop_path_ratio) if drop_path_ratio > 0.0 else nn.Identity()
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.linear = Mlp(dim, 0)
        self.attention = EarthAttention3D(dim, heads, 0, self.window_size, device=device)
        self.padding_front, self.padding_back = 0, 5
        self.type_of_windows = self.attention.type_of_windows

    def forward(self, x, Z, H, W, roll, out=None):
        assert_plain_tree(self, "EarthSpecificBlock")
        return fused.earth_block(self, x, Z, H, W, roll, out=out)

    def gen_mask(self, x):
        """reference layers.py:153-181: the shifted-window attention mask for a padded activation `x` (1, Z, Hp, W, C) ->
        (W/12, types, 144, 144) fp32 in {0, -100}.  The attention kernels never materialise it (closed form per lane,
        csrc/common.h win_mask); this returns the same kernel-side closed form, exported by `pangu_window_mask_export`
        (bit-exact against the reference's slicing construction, tests/test_gpu_parity.py), expanded over the longitude
        windows as the reference's tensor is (its values do not depend on the longitude window: no W slicing)."""
        from . import ops
        _, Z, Hp, W, _ = x.shape
        m = ops.window_mask(Z, Hp - self.padding_back - self.padding_front, W, x.device)      # (types, 144, 144)
        return m.unsqueeze(0).expand(W // self.window_size[2], -1, -1, -1)


class EarthSpecificLayer(nn.Module):
    """reference layers.py:96-125.  `use_checkpoint` is accepted for signature parity and ignored: with the
    fused attention nothing of size (..,144,144) is kept, so activations fit HBM without recompute."""

    def __init__(self, depth, dim, drop_path_ratio_list, heads, use_checkpoint=False, device=None):
        super().__init__()
        self.device = device
        self.depth = depth
        blocks = OrderedDict()
        for i in range(depth):
            blocks[f"EarthSpecificBlock{i}"] = EarthSpecificBlock(dim, drop_path_ratio_list[i], heads, device=device)
        self.blocks = nn.Sequential(blocks)
        self.use_checkpoint = use_checkpoint

    def forward(self, x, Z, H, W, out=None):
        n = len(self.blocks)
        for i, blk in enumerate(self.blocks):
            x = blk(x, Z, H, W, roll=(i % 2 == 1), out=out if i == n - 1 else None)
        return x


class DownSample(nn.Module):
    """reference layers.py:423-459."""

    # frozen fp32 inference: its projections on the exact-split bf16-MFMA kernel (PanguModel.use_split_projections sets it)
    split_projections = True

    def __init__(self, dim):
        super().__init__()
        self.linear = nn.Linear(in_features=4 * dim, out_features=2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)

    def forward(self, x, Z, H, W):
        return fused.down_sample(self, x, Z, H, W)


class UpSample(nn.Module):
    """reference layers.py:461-499."""

    # frozen fp32 inference: its projections on the exact-split bf16-MFMA kernel (PanguModel.use_split_projections sets it)
    split_projections = True

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.linear1 = nn.Linear(input_dim, output_dim * 4, bias=False)
        self.linear2 = nn.Linear(output_dim, output_dim, bias=False)
        self.norm = nn.LayerNorm(output_dim)

    def forward(self, x, Z=8, H2=None, W2=None, H=None):
        if H2 is None:       # the reference's forward(x): on its grid, W2 = 2 (H2 - 1) less one latitude row (layers.py:480-489)
            H2 = (1 + math.isqrt(1 + 2 * (x.shape[1] // Z))) // 2
            W2, H = 2 * (H2 - 1), 2 * H2 - 1
        if Z * H2 * W2 != x.shape[1]:
            raise RuntimeError(f"UpSample: {x.shape[1]} tokens are not a ({Z}, {H2}, {W2}) grid; pass Z, H2, W2, H")
        return fused.up_sample(self, x, Z, H2, W2, H)


class PatchRecovery_pretrain(nn.Module):
    """reference layers.py:501-545."""

    # frozen fp32 inference: its projections on the exact-split bf16-MFMA kernel (PanguModel.use_split_projections sets it)
    split_projections = True

    def __init__(self, dim):
        super().__init__()
        self.patch_size = (2, 4, 4)
        self.dim = dim
        self.conv = nn.Conv1d(in_channels=dim, out_channels=160, kernel_size=1, stride=1)
        self.conv_surface = nn.Conv1d(in_channels=dim, out_channels=64, kernel_size=1, stride=1)

    def forward(self, x, Z, H, W):
        return fused.patch_recover(self, x, Z, H, W)
