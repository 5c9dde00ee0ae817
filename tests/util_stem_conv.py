"""Shared inputs, float64 references and error bounds for the tests of
the stem conv kernels (``machin_amd/ops/hip/conv1_wrw.hip``):
``Conv2d(4, 32, 8, stride=4)`` on ``[B, 84, 84, 4]`` u8 frames.

Everything here runs on the CPU. Everything returned from the cached
functions is shared between tests: do not modify it in place.

The kernels multiply ``bf16(float32(v) * float32(scale))`` (the
dequantised byte, :func:`dequant`) with the bf16 weight (forward) or the
bf16 ``dy`` (weight gradient) and accumulate in fp32. The references
take exactly these operands to float64.

Exact kinds. Every product and every partial sum is an integer multiple
of ``scale`` below ``2^24 * scale``, so fp32 accumulation is exact in
any order and the result must equal the reference bit for bit. They run
at ``scale`` 1 and 2^-8; both dequantise every byte exactly. At 2^-8 the
bias is the same integer times ``scale``: the case is the scale-1 case
in units of 2^-8, so every property below (values exact in bf16, exact
zeros, exact ties) holds at both scales, and the reference at 2^-8 is
the reference at 1 times 2^-8. A kernel that ignores ``scale``, or
applies it to anything but the byte, passes at 1 only.

``taps0`` .. ``taps7``
    one-hot weights: in set ``s`` output channel ``c`` has a single 1 at
    patch index ``n = s * 32 + c`` (``n = (ky * 8 + kx) * 4 + ci``), so
    the 8 sets cover all 256 taps. Frames are full-range random bytes
    with 0, 127, 128 and 255 forced into every frame, bias in
    {-1, 0, 1}: the output is the pixel itself plus the bias.
``signs``
    frames in {0, 1}, weights in {-1, 0, 1}, bias in -2..2: small
    outputs of both signs, all exact in bf16, with exact zeros.
``dense``
    frames 0..255, weights and bias in -3..3: the accumulator is an
    exact integer too large for bf16, so the one round-to-nearest-even of
    the epilogue is tested, exact ties included (the builder reseeds
    until ties occur with and without the bias).
weight gradient ``int``
    ``dy`` in -2..2, frames 0..255, masks ``none`` / ``random`` /
    ``clear`` / ``set`` / ``from_forward`` (the mask of the ``signs``
    forward at scale 1).

Rounding kind (``round``): random bytes, weights ``randn * 0.05``
rounded to bf16, bias ``randn * 0.1``, ``dy = bf16(randn * 0.1)``,
scale 1/255. Per element

    |got - ref| <= F * (K + 8) * 2^-24 * S  (+ 2^-8 |ref| if bf16 output)

with ``S`` the sum of the absolute values of the element's terms and
``K`` its reduction length (256 forward, 400 * B weight gradient): the
form of ``util_noisy_linear.reference64`` times ``F``. ``F`` covers the
adds inside ``v_mfma_f32_16x16x32_bf16``, which the NoisyLinear kernels
that carry the ``F = 1`` form do not use. Each fp32 add rounded to
nearest is off by at most 2^-24 of its result; an adder that truncates
instead is off by at most 2^-23, twice as much, which would give
``F = 2``. ``F`` is not fitted to the conv kernels. It is checked on
the instruction alone: ``test_stem_conv_gpu.py`` runs
``ext.mfma_probe`` (one MFMA, no kernel logic) on random bf16 tiles
(:func:`probe_tiles`) and asserts ``|err| <= F_MFMA * 2^-24 * S`` per
element. Measured on an MI355X, worst ``|err| / (S * 2^-24)`` of one
instruction (``MFMA_PROBE_MEASURED``): 3.359 over all tiles; by family
1.126 (normal), 3.359 (exponents spread over 2^-6..2^6 inside one sum),
2.171 (all positive), 0 (values in [1, 2): the sums fit in 24 bits).
That is more than 2: the instruction is not a chain of truncating fp32
adds (it loses the low bits of small products against the largest one),
so ``F_MFMA`` is the next power of two above the measurement, 4. The
bias gradient is summed with ordinary fp32 adds and keeps ``F = 1``.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import torch as t
import torch.nn.functional as F

BATCHES = (1, 3, 5)
EXACT_SCALES = (1.0, 2.0 ** -8)
FWD_EXACT_KINDS = tuple(f"taps{s}" for s in range(8)) + ("signs", "dense")
MASK_KINDS = ("none", "random", "clear", "set", "from_forward")
FORCED_BYTES = (0, 127, 128, 255)
# 1/255 as the kernels receive it: a float32
ROUND_SCALE = float(t.tensor(1.0 / 255.0, dtype=t.float32))
# see the module docstring
F_MFMA = 4
# worst |err| / (S * 2^-24) of one v_mfma_f32_16x16x32_bf16 over
# probe_tiles(), measured on an MI355X (per-instruction constant)
MFMA_PROBE_MEASURED = 3.359

OHW, POS, TAPS, COUT = 20, 400, 256, 32


def scale_tensor(scale):
    return t.tensor(scale, dtype=t.float32)


def dequant(frames, scale):
    """bf16(float32(v) * float32(scale)) of u8 ``frames``."""
    return (frames.to(t.float32) * scale_tensor(scale)).to(t.bfloat16)


def repack(weight):
    """[32, 4, 8, 8] conv weight -> patch-major [256, 32], row
    ``n = (ky * 8 + kx) * 4 + ci`` (the expression of ``_FusedConv1Fn``)."""
    return weight.permute(2, 3, 1, 0).reshape(256, 32)


def tap_index(ky, kx, ci):
    return (ky * 8 + kx) * 4 + ci


def round_bf16(x, ties_away=False):
    """float64 tensor rounded ONCE to the nearest bf16 value (8
    significand bits), ties to even (or away from zero), as float64."""
    m, e = np.frexp(x.numpy())          # x = m * 2^e, 0.5 <= |m| < 1
    v = np.ldexp(m, 8)                  # 128 <= |v| < 256
    if ties_away:
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    else:
        r = np.rint(v)                  # half to even
    return t.from_numpy(np.ldexp(r, e - 8))


def is_bf16_tie(x):
    """True where a float64 value lies exactly halfway between two
    neighbouring bf16 values."""
    m, _ = np.frexp(x.numpy())
    v = np.abs(np.ldexp(m, 8))
    return t.from_numpy(v - np.floor(v) == 0.5)


def pack_mask(pos):
    """[K, 32] bool -> [K] int32, bit c of word k = pos[k, c]."""
    w = (pos.to(t.int64) << t.arange(32, dtype=t.int64)).sum(dim=1)
    return t.where(w >= 2 ** 31, w - 2 ** 32, w).to(t.int32)


def unpack_mask(mask):
    """[K] int32 words -> [K, 32] bool, bit c of word k at [k, c]."""
    shifts = t.arange(32, device=mask.device, dtype=t.int32)
    return ((mask.view(-1, 1) >> shifts) & 1).bool()


def rows(y):
    """[B, 32, 20, 20] -> the kernels' [B * 400, 32] (NHWC rows)."""
    return y.permute(0, 2, 3, 1).reshape(-1, COUT)


def im2col(x):
    """[B, 84, 84, 4] values -> [B * 400, 256] float64 patch rows in the
    kernels' order: row ``(b * 20 + oh) * 20 + ow``, column
    ``(ky * 8 + kx) * 4 + ci``."""
    B = x.shape[0]
    cols = F.unfold(x.double().permute(0, 3, 1, 2), 8, stride=4)
    cols = cols.view(B, 4, 8, 8, POS).permute(0, 4, 2, 3, 1)
    return cols.reshape(B * POS, TAPS)


def _ints(gen, lo, hi, *size):
    return t.randint(lo, hi + 1, size, generator=gen)


def _force_bytes(frames, gen):
    """Put each of FORCED_BYTES at a random place of every frame."""
    flat = frames.view(frames.shape[0], -1)
    for b in range(flat.shape[0]):
        at = t.randperm(flat.shape[1], generator=gen)[:len(FORCED_BYTES)]
        flat[b, at] = t.tensor(FORCED_BYTES, dtype=t.uint8)
    return frames


def _forward_inputs(batch, kind, seed):
    """(frames u8 NHWC, weight fp32 [32, 4, 8, 8], integer or real bias)
    before scaling."""
    gen = t.Generator().manual_seed(seed)
    shape = (batch, 84, 84, 4)
    if kind.startswith("taps"):
        s = int(kind[4:])
        frames = _force_bytes(_ints(gen, 0, 255, *shape).to(t.uint8), gen)
        w_rs = t.zeros(TAPS, COUT)
        for c in range(COUT):
            w_rs[s * 32 + c, c] = 1.0
        # inverse of repack()
        weight = w_rs.view(8, 8, 4, 32).permute(3, 2, 0, 1).contiguous()
        bias = _ints(gen, -1, 1, COUT).float()
    elif kind == "signs":
        frames = _ints(gen, 0, 1, *shape).to(t.uint8)
        weight = _ints(gen, -1, 1, 32, 4, 8, 8).float()
        bias = _ints(gen, -2, 2, COUT).float()
    elif kind == "dense":
        frames = _ints(gen, 0, 255, *shape).to(t.uint8)
        weight = _ints(gen, -3, 3, 32, 4, 8, 8).float()
        bias = _ints(gen, -3, 3, COUT).float()
    else:
        assert kind == "round", kind
        frames = _ints(gen, 0, 255, *shape).to(t.uint8)
        weight = (t.randn(32, 4, 8, 8, generator=gen) * 0.05).to(
            t.bfloat16).float()
        bias = t.randn(COUT, generator=gen) * 0.1
    return frames, weight, bias


def _forward_terms(frames, weight, bias, scale):
    """float64 ``acc`` and sum of absolute terms ``S`` (without bias) as
    [K, 32] rows, from the operands the kernel multiplies."""
    x = dequant(frames, scale).double().permute(0, 3, 1, 2)
    w = weight.to(t.bfloat16).double()
    acc = rows(F.conv2d(x, w, stride=4))
    s = rows(F.conv2d(x.abs(), w.abs(), stride=4))
    return acc, s


@functools.lru_cache(maxsize=None)
def forward_case(batch, kind, scale):
    """Inputs of a forward case: ``frames`` u8 [B, 84, 84, 4],
    ``weight`` fp32 [32, 4, 8, 8] (exact in bf16), ``bias`` fp32 [32],
    ``scale``. The taps sets share their frames and bias."""
    exact = kind != "round"
    assert scale in EXACT_SCALES if exact else scale == ROUND_SCALE
    base = 1000 * batch + (0 if kind.startswith("taps")
                           else 100 + FWD_EXACT_KINDS.index(kind)
                           if exact else 200)
    for seed in itertools.count(base, 17):
        frames, weight, bias = _forward_inputs(batch, kind, seed)
        if kind != "dense":
            break
        # ties of the epilogue's rounding must occur, with and without
        # the bias; reseed until they do
        acc, _ = _forward_terms(frames, weight, bias, 1.0)
        if bool(is_bf16_tie(acc).any()) and \
                bool(is_bf16_tie(acc + bias.double()).any()):
            break
    if exact:
        bias = bias * scale   # a power of two: exact
    return SimpleNamespace(frames=frames, weight=weight, bias=bias,
                           scale=scale, kind=kind, batch=batch)


def forward_reference(batch, kind, scale, with_bias=True):
    return _forward_reference(batch, kind, scale, bool(with_bias))


@functools.lru_cache(maxsize=None)
def _forward_reference(batch, kind, scale, with_bias):
    """float64 reference of a forward case, as [K, 32] rows / [K] words:
    ``pre`` = acc + bias, ``s`` = sum of absolute terms (|bias|
    included), ``y`` = pre rounded once to bf16, ``relu`` its ReLU (both
    bf16 tensors), ``mask`` the packed ``y > 0``, and ``bound`` the
    rounding bound of the module docstring (for ``y`` and ``relu``)."""
    case = forward_case(batch, kind, scale)
    acc, s = _forward_terms(case.frames, case.weight, case.bias, scale)
    if with_bias:
        b = case.bias.double()
        acc, s = acc + b, s + b.abs()
    y64 = round_bf16(acc)
    y = y64.to(t.bfloat16)
    assert t.equal(y.double(), y64)
    bound = F_MFMA * (TAPS + 8) * 2.0 ** -24 * s + 2.0 ** -8 * acc.abs()
    return SimpleNamespace(pre=acc, s=s, y=y, relu=t.relu(y),
                           mask=pack_mask(y > 0), bound=bound)


@functools.lru_cache(maxsize=None)
def wrw_case(batch, kind, scale):
    """Inputs of a weight-gradient case: ``frames`` u8 [B, 84, 84, 4]
    and ``dy`` bf16 [B * 400, 32]; ``kind`` is ``int`` or ``round``."""
    gen = t.Generator().manual_seed(7000 + 10 * batch + (kind == "int"))
    frames = _ints(gen, 0, 255, batch, 84, 84, 4).to(t.uint8)
    if kind == "int":
        assert scale in EXACT_SCALES
        dy = _ints(gen, -2, 2, batch * POS, COUT).to(t.bfloat16)
    else:
        assert kind == "round" and scale == ROUND_SCALE
        dy = (t.randn(batch * POS, COUT, generator=gen) * 0.1).to(
            t.bfloat16)
    return SimpleNamespace(frames=frames, dy=dy, scale=scale, kind=kind,
                           batch=batch)


@functools.lru_cache(maxsize=None)
def wrw_mask(batch, mask_kind):
    """[B * 400] int32 packed mask, or None for ``none``."""
    K = batch * POS
    if mask_kind == "none":
        return None
    if mask_kind == "random":
        gen = t.Generator().manual_seed(7100 + batch)
        return pack_mask(t.randint(0, 2, (K, COUT), generator=gen).bool())
    if mask_kind == "clear":
        return t.zeros(K, dtype=t.int32)
    if mask_kind == "set":
        return t.full((K,), -1, dtype=t.int32)
    assert mask_kind == "from_forward", mask_kind
    return forward_reference(batch, "signs", 1.0, True).mask


def wrw_float64(frames, dy, mask, scale):
    """``(grad_w [32, 4, 8, 8], grad_b [32], s_w, s_b)`` in float64 from
    the operands the kernels multiply: ``dequant(frames)`` and the masked
    bf16 ``dy``; ``s_*`` are the sums of the absolute terms."""
    batch = frames.shape[0]
    x = dequant(frames, scale).double()
    cols = F.unfold(x.permute(0, 3, 1, 2), 8, stride=4)  # [B, 256, 400]
    d = dy.double()
    if mask is not None:
        d = d * unpack_mask(mask).double()
    d = d.view(batch, POS, COUT)
    gw = t.einsum("bpo,bnp->on", d, cols).view(32, 4, 8, 8)
    sw = t.einsum("bpo,bnp->on", d.abs(), cols.abs()).view(32, 4, 8, 8)
    return gw, d.sum(dim=(0, 1)), sw, d.abs().sum(dim=(0, 1))


def wrw_reference(batch, kind, scale, mask_kind="none"):
    return _wrw_reference(batch, kind, scale, mask_kind)


@functools.lru_cache(maxsize=None)
def _wrw_reference(batch, kind, scale, mask_kind):
    """float64 reference of a weight-gradient case with the rounding
    bounds of the module docstring (``K = 400 * B``; the bias gradient
    is summed without the MFMA: ``F = 1``)."""
    case = wrw_case(batch, kind, scale)
    gw, gb, sw, sb = wrw_float64(case.frames, case.dy,
                                 wrw_mask(batch, mask_kind), scale)
    k = POS * batch + 8
    return SimpleNamespace(
        grad_w=gw, grad_b=gb, s_w=sw, s_b=sb,
        bound_w=F_MFMA * k * 2.0 ** -24 * sw, bound_b=k * 2.0 ** -24 * sb,
    )


def worst_ratio(got, ref, bound):
    """Largest ``|got - ref| / bound``; elements whose bound is zero
    must match exactly."""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert bool(t.isfinite(g).all())
    err = (g - ref).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all())
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


@functools.lru_cache(maxsize=None)
def probe_tiles(count=64):
    """Random bf16 operands of ``ext.mfma_probe``: ``A [count, 16, 32]``
    and ``B [count, 32, 16]``, a quarter each of normal values, normal
    values times 2^(-6..6) per element (wide exponent spread inside one
    sum), positive values (no cancellation: the sum is as large as S) and
    values in [1, 2) (every product needs 16 significand bits)."""
    gen = t.Generator().manual_seed(99)
    q = count // 4

    def normal(*size):
        return t.randn(*size, generator=gen)

    def spread(*size):
        return normal(*size) * 2.0 ** _ints(gen, -6, 6, *size).float()

    def positive(*size):
        return normal(*size).abs()

    def dense_bits(*size):
        return 1 + t.rand(*size, generator=gen)

    a, b = [], []
    for make in (normal, spread, positive, dense_bits):
        a.append(make(q, 16, 32))
        b.append(make(q, 32, 16))
    return t.cat(a).to(t.bfloat16), t.cat(b).to(t.bfloat16)
