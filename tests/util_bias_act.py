"""Plain reference, inputs and bounds for the tests of the fused
bias + ReLU kernels (``machin_amd/ops/hip/bias_act.hip``).

Everything here runs on the CPU with numpy and never imports the
extension. Everything returned from the cached functions is shared
between tests: do not modify it in place.

bf16 is handled as raw 16-bit patterns (``uint16`` arrays). Widening to
fp32 is a 16-bit shift (:func:`widen`), narrowing is round-to-nearest-
even in integer arithmetic (:func:`narrow` from fp32, :func:`narrow64`
from float64 without the double rounding a detour over fp32 would add).
NaN stays NaN. Neither ``torch.relu``, ``Tensor.to(bfloat16)`` nor
``threshold_backward`` is used.

Forward (:func:`forward`): the fp32 bias is narrowed to bf16, widened,
added to the widened activation in IEEE fp32 (numpy ``float32``; no
float64, the kernel rounds twice and so must the reference), the sum is
narrowed to bf16, then ``s > 0 ? s : (isnan(s) ? s : +0)``.

Backward (:func:`backward`): ``gx = (act <= 0) ? +0 : gy``, so a NaN
activation passes ``gy`` through; the bias gradient is the float64 sum
of ``gx`` over the rows.

Flat variants: the same values, moved between the NHWC rows ``[N*HW,
C]`` and the NCHW-flat matrix ``[N, C*HW]`` by the index map of
:func:`flat_index`, written out element by element.

Exact bias gradient (:func:`exact_case`). ``gy`` is a non-zero integer
in +-{1, 2, 3} everywhere, with seeded signs. Row ``r`` is live
(``act > 0``) in the one channel ``c`` with ``(r + c) % C == 0``, where
``gy`` is +-1, and dead (``act`` in {+0, -0, -1, -1000}) everywhere
else. So every row contributes exactly +-1 to exactly one channel,
every dead position carries a gradient that would show if it leaked,
and every partial sum of any grouping is an integer below 2^24, exact
in fp32. A channel total is a sum of about ``R / C`` seeded signs;
:func:`exact_preconditions` asserts ``|total| <= 256`` (all integers up
to 256 are bf16 values, so the final rounding is the identity) and that
every row is lit. With both, one lost, repeated or misattributed row
changes a total by at least 1 and the kernel must equal the float64 sum
exactly.

Rounding bound (:func:`grad_interval`). The kernels sum ``n`` fp32
terms per channel (one per row, zeros included) in a fixed order of
their own and round once to bf16. Any order of fp32 additions is off by
at most ``e = (n - 1) 2^-24 sum|gx|`` (Jeannerod and Rump, 2013: the
first-order bound holds without higher-order terms), and rounding is
monotone, so the result lies in ``[rne(ref - e), rne(ref + e)]`` with
``ref`` the float64 sum. Nothing in it is measured.
"""
import functools

import numpy as np

U16 = np.uint16
POS_ZERO = U16(0x0000)
NEG_ZERO = U16(0x8000)


# ---- bf16 as bit patterns ---------------------------------------------
def widen(bits):
    """uint16 bf16 patterns -> the float32 values they denote."""
    bits = np.asarray(bits, dtype=U16)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow(x):
    """float32 -> uint16 bf16 patterns, round to nearest, ties to even,
    in integer arithmetic. A NaN gives a quiet NaN of the same sign."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    lsb = (u >> np.uint64(16)) & np.uint64(1)
    r = (u + np.uint64(0x7FFF) + lsb) >> np.uint64(16)
    r = np.where(nan, (u >> np.uint64(16)) | np.uint64(0x0040), r)
    return r.astype(U16)


def narrow64(x):
    """float64 -> uint16 bf16 patterns, one rounding to nearest even.

    The magnitude is truncated to bf16 (truncations compose, so going
    through fp32 is harmless there), then the nearer of that value and
    its upper neighbour is chosen in float64, where both differences are
    exact; 2^128 stands in for the neighbour of the largest finite."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nan = np.isnan(x)
    ax = np.abs(np.where(nan, 0.0, x))
    with np.errstate(over="ignore"):
        f = ax.astype(np.float32)
    over = f.astype(np.float64) > ax
    f = np.where(over, np.nextafter(f, np.float32(0.0)), f)
    f = f.astype(np.float32)
    lo = (f.view(np.uint32) >> np.uint32(16)).astype(np.uint32)
    hi = lo + np.uint32(1)
    with np.errstate(invalid="ignore"):       # inf + 1 is a NaN pattern
        lo_v = widen(lo.astype(U16)).astype(np.float64)
        hi_v = widen(hi.astype(U16)).astype(np.float64)
    hi_v = np.where(np.isinf(hi_v), 2.0 ** 128, hi_v)
    inf_in = np.isinf(ax)
    with np.errstate(invalid="ignore"):
        d_lo = np.where(inf_in, 0.0, ax - lo_v)
        d_hi = np.where(inf_in, 1.0, hi_v - ax)
    up = (d_hi < d_lo) | ((d_hi == d_lo) & ((lo & np.uint32(1)) == 1))
    mag = np.where(up, hi, lo).astype(np.uint32)
    sign = np.where(np.signbit(x), np.uint32(0x8000), np.uint32(0))
    out = (mag | sign).astype(U16)
    return np.where(nan, U16(0x7FC0), out).astype(U16)


def is_nan_bits(bits):
    return (np.asarray(bits, dtype=U16) & U16(0x7FFF)) > U16(0x7F80)


def assert_same_bits(got, ref, what):
    """Equal patterns; a NaN only has to be a NaN in the same place."""
    got, ref = np.asarray(got, dtype=U16), np.asarray(ref, dtype=U16)
    assert got.shape == ref.shape, f"{what}: {got.shape} != {ref.shape}"
    got_nan, ref_nan = is_nan_bits(got), is_nan_bits(ref)
    assert np.array_equal(got_nan, ref_nan), f"{what}: NaN positions"
    bad = (got != ref) & ~ref_nan
    assert not bad.any(), (
        f"{what}: {bad.sum()} differ, first at "
        f"{tuple(int(i) for i in np.argwhere(bad)[0])}: "
        f"{got[bad][0]:#06x} != {ref[bad][0]:#06x}")


def bits_of(values):
    """bf16 patterns of values that are exact in bf16."""
    v = np.asarray(values, dtype=np.float32)
    b = narrow(v)
    assert np.array_equal(widen(b), v, equal_nan=True), "not exact in bf16"
    return b


# ---- the operations ----------------------------------------------------
def forward_sum(y_bits, bias):
    """The fp32 sum ``float(y) + float(bf16(bias[c]))`` of the forward,
    before its narrowing. ``y_bits`` is ``[R, C]``, ``bias`` fp32 ``[C]``."""
    b = widen(narrow(np.asarray(bias, dtype=np.float32)))
    with np.errstate(over="ignore", invalid="ignore"):
        return (widen(y_bits) + b[None, :]).astype(np.float32)


def relu_bits(s_bits):
    s = widen(s_bits)
    with np.errstate(invalid="ignore"):
        keep = (s > 0) | is_nan_bits(s_bits)
    return np.where(keep, s_bits, POS_ZERO).astype(U16)


def forward(y_bits, bias):
    """relu(bf16(float(y) + float(bf16(bias)))) as bf16 patterns."""
    return relu_bits(narrow(forward_sum(y_bits, bias)))


def backward(gy_bits, act_bits):
    """(gx patterns ``[R, C]``, float64 bias gradient ``[C]``)."""
    with np.errstate(invalid="ignore"):
        dead = widen(act_bits) <= 0
    gx = np.where(dead, POS_ZERO, np.asarray(gy_bits, dtype=U16)).astype(U16)
    with np.errstate(invalid="ignore", over="ignore"):
        gb = widen(gx).astype(np.float64).sum(axis=0)
    return gx, gb


def flat_index(N, C, HW):
    """(row, col), each ``[N, C*HW]``: element ``[n, c*HW + hw]`` of the
    NCHW-flat matrix is element ``[n*HW + hw, c]`` of the NHWC rows."""
    n = np.arange(N, dtype=np.int64)[:, None, None]
    c = np.arange(C, dtype=np.int64)[None, :, None]
    hw = np.arange(HW, dtype=np.int64)[None, None, :]
    row = np.broadcast_to(n * HW + hw, (N, C, HW)).reshape(N, C * HW)
    col = np.broadcast_to(c, (N, C, HW)).reshape(N, C * HW)
    return row, col


def rows_to_flat(rows, N):
    R, C = rows.shape
    assert R % N == 0
    row, col = flat_index(N, C, R // N)
    return np.ascontiguousarray(rows[row, col])


def flat_to_rows(flat, C):
    N, L = flat.shape
    assert L % C == 0
    HW = L // C
    row, col = flat_index(N, C, HW)
    rows = np.empty((N * HW, C), dtype=flat.dtype)
    rows[row, col] = flat
    return rows


def forward_flat(y_bits, bias, N):
    return rows_to_flat(forward(y_bits, bias), N)


def backward_flat(gy_flat_bits, act_flat_bits, C):
    """NCHW-flat gradient and activation -> (gx as NHWC rows, float64
    bias gradient)."""
    return backward(flat_to_rows(gy_flat_bits, C),
                    flat_to_rows(act_flat_bits, C))


# ---- every bf16 value ---------------------------------------------------
TABLE_C = 64
TABLE_N, TABLE_HW = 128, 512   # 65536 rows as samples: C*HW = 32768


def all_patterns(C=TABLE_C):
    """[65536, C]: row r holds pattern r in every channel."""
    return np.repeat(np.arange(65536, dtype=np.uint32).astype(U16)[:, None],
                     C, axis=1)


@functools.lru_cache(maxsize=None)
def edge_bias():
    """64 fp32 bias values: the edges first, seeded ordinary values
    after them."""
    f32 = np.float32
    tie = f32(1.0) + f32(2.0 ** -8)           # between 1 and 1 + 2^-7
    tie3 = f32(1.0) + f32(3 * 2.0 ** -8)      # rounds up, to the even side
    edges = [
        0.0, -0.0, 1.0, -1.0, 0.1, -0.1, 1.0 / 3.0, 3.14159265,
        tie, np.nextafter(tie, f32(0)), np.nextafter(tie, f32(2)),
        tie3, np.nextafter(tie3, f32(0)), np.nextafter(tie3, f32(2)),
        -tie, -tie3,
        2.0 ** -126, -(2.0 ** -126),          # smallest normal
        2.0 ** -130, -(2.0 ** -130),          # a bf16 subnormal
        2.0 ** -140,                          # fp32 subnormal, bf16 zero
        2.0 ** -126 * (1 - 2.0 ** -9),        # subnormal, narrows to normal
        3.0e38, -3.0e38,                      # sums overflow to inf
        np.finfo(f32).max,                    # narrows to inf
        np.inf, -np.inf, np.nan,
        256.0, -65280.0, 1.0e-20, -7.0e20,
    ]
    rng = np.random.default_rng(64)
    rest = rng.standard_normal(TABLE_C - len(edges)) * 2.0
    out = np.concatenate([np.array(edges, dtype=f32), rest.astype(f32)])
    assert out.shape == (TABLE_C,)
    return out


@functools.lru_cache(maxsize=None)
def table_forward():
    """(y patterns, bias, fp32 sum, reference output) of the forward on
    every bf16 value against :func:`edge_bias`."""
    y = all_patterns()
    bias = edge_bias()
    s = forward_sum(y, bias)
    return y, bias, s, relu_bits(narrow(s))


def subnormal_f32(x):
    ax = np.abs(x)
    return (ax > 0) & (ax < np.float32(2.0 ** -126))


@functools.lru_cache(maxsize=None)
def edge_gy():
    """64 bf16 gradient values, one per channel: the first 8 channels
    are not finite, the others are."""
    f32 = np.float32
    head = [np.inf, -np.inf, np.nan, -np.nan, np.inf, np.nan, -np.inf,
            np.inf]
    finite = [0.0, -0.0, 1.0, -2.0, 0.5, -0.75, 3.0, 2.0 ** -130,
              -(2.0 ** -126), 1.0e-3, -250.0, 96.0]
    rng = np.random.default_rng(65)
    rest = rng.standard_normal(TABLE_C - len(head) - len(finite))
    vals = np.array(head + finite + list(rest), dtype=f32)
    bits = narrow(vals)
    bits[3] = U16(0xFFC0)                     # a NaN with the sign set
    return bits


@functools.lru_cache(maxsize=None)
def table_backward():
    """(gy patterns, act patterns, gx reference, float64 bias gradient)
    with every bf16 value as the activation."""
    act = all_patterns()
    gy = np.ascontiguousarray(
        np.broadcast_to(edge_gy()[None, :], act.shape))
    gx, gb = backward(gy, act)
    return gy, act, gx, gb


# ---- exact bias gradient ------------------------------------------------
def rows_per_pass(C):
    return 256 // (C // 8)


def _row_shapes():
    shapes = []
    for C in (8, 24, 64, 136, 320, 2048):
        RP = rows_per_pass(C)
        for R in (1, RP - 1, RP, RP + 1, 2 * RP + 1):
            if R >= 1 and (R, C) not in shapes:
                shapes.append((R, C))
    shapes += [(4099, 64), (2048 * 32 + 1, 64), (65573, 64), (131109, 64)]
    return shapes


# (R, C) of the row kernels; R = 0 has a test of its own
EXACT_ROW_SHAPES = _row_shapes()
# (N, C, HW) of the flat kernels
EXACT_FLAT_SHAPES = (
    [(N, 64, 49) for N in (1, 3, 2047, 2048, 2049, 4097)]
    + [(5, 8, 1), (4, 24, 15), (3, 64, 512), (2, 2048, 16), (3, 320, 9)]
)

_LIVE = bits_of([0.5, 1.0, 7.0, 1000.0])
_DEAD = bits_of([0.0, -0.0, -1.0, -1000.0])
_MAG = bits_of([1.0, 2.0, 3.0])
SIGN_BIT = U16(0x8000)


@functools.lru_cache(maxsize=4)
def exact_case(R, C):
    """(gy patterns, act patterns) of the exact bias-gradient case, both
    ``[R, C]`` (see the module docstring)."""
    rng = np.random.default_rng(R * 4099 + C)
    gy = _MAG[rng.integers(0, 3, (R, C))]
    gy = gy | np.where(rng.integers(0, 2, (R, C)) == 1, SIGN_BIT, U16(0))
    act = _DEAD[rng.integers(0, 4, (R, C))]
    r = np.arange(R, dtype=np.int64)
    c = (-r) % C                              # (r + c) % C == 0
    act[r, c] = _LIVE[rng.integers(0, 4, R)]
    gy[r, c] = (gy[r, c] & SIGN_BIT) | _MAG[0]
    return gy.astype(U16), act.astype(U16)


def exact_preconditions(gy, act):
    """Asserts what makes the bias gradient of :func:`exact_case` exact
    and returns (gx reference, float64 totals). Reference only."""
    R, C = gy.shape
    gx, total = backward(gy, act)
    g = widen(gy)
    assert np.all(g != 0) and np.all(g == np.round(g)), "gy integer, != 0"
    assert np.all(np.abs(g) <= 3)
    live = widen(act) > 0
    lit = live & (widen(gx) != 0)
    assert np.all(lit.sum(axis=1) >= 1), "a row without a live element"
    assert np.all(live.sum(axis=1) < C), "a row without a dead element"
    assert np.all(total == np.round(total))
    assert np.all(np.abs(total) <= 256), np.abs(total).max()
    # what the test needs from them: the totals are bf16 values
    assert np.array_equal(widen(narrow64(total)).astype(np.float64), total)
    return gx, total


# ---- rounding bound -----------------------------------------------------
ROUND_ROW_SHAPES = [(513, 8), (171, 24), (4099, 64), (65573, 64),
                    (31, 136), (4099, 320), (3, 2048)]
ROUND_FLAT_SHAPES = [(2049, 64, 49), (4, 24, 15), (3, 320, 9)]


@functools.lru_cache(maxsize=4)
def random_case(R, C):
    """(y patterns, fp32 bias, gy patterns) of ordinary ``randn`` values."""
    rng = np.random.default_rng(R * 31 + C)
    y = narrow(rng.standard_normal((R, C)).astype(np.float32))
    bias = (rng.standard_normal(C) * 0.5).astype(np.float32)
    gy = narrow(rng.standard_normal((R, C)).astype(np.float32))
    return y, bias, gy


def grad_interval(gx_bits):
    """(lo, hi, ref, e), float64 ``[C]``: the bias gradient of a kernel
    that sums the rows of ``gx`` in fp32 in any order and rounds once to
    bf16 lies in ``[lo, hi]``."""
    g = widen(gx_bits).astype(np.float64)
    n = g.shape[0]
    ref = g.sum(axis=0)
    e = max(n - 1, 0) * 2.0 ** -24 * np.abs(g).sum(axis=0)
    lo = widen(narrow64(ref - e)).astype(np.float64)
    hi = widen(narrow64(ref + e)).astype(np.float64)
    return lo, hi, ref, e


def check_grad_interval(got, gx_bits, what):
    """Asserts ``got`` (float array ``[C]``) against :func:`grad_interval`
    after printing the worst ``|got - ref| / e``."""
    got = np.asarray(got, dtype=np.float64)
    lo, hi, ref, e = grad_interval(gx_bits)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(e > 0, np.abs(got - ref) / e, 0.0)
    print(f"{what}: worst |got - ref| / e = {ratio.max():.4f}")
    assert np.array_equal(widen(narrow64(got)).astype(np.float64), got), \
        f"{what}: not bf16-rounded"
    bad = ~((got >= lo) & (got <= hi))
    assert not bad.any(), (
        f"{what}: channels {np.nonzero(bad)[0][:8]} outside "
        f"[{lo[bad][:4]}, {hi[bad][:4]}]: {got[bad][:4]}")
