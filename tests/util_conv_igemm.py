"""Cases and the float64 CPU reference shared by the implicit-GEMM conv
tests (test_conv_igemm_gpu.py, test_conv_igemm_cpu.py)."""
import functools
from types import SimpleNamespace

import torch as t
import torch.nn.functional as F

# name -> (Cin, Cout, kernel, stride)
GEOMETRY = {"conv2": (32, 64, 4, 2), "conv3": (64, 64, 3, 1)}

# (geometry, N, H, W, flatten, MACHIN_CONV_IGEMM_WG or None)
CASES = [
    # one output pixel: a single partial tile
    ("conv2", 1, 4, 4, False, None),
    # 2x3 outputs; (H - KH) % 2 != 0, so input row 6 has dx == 0; four
    # ragged parity classes (4x5 .. 3x4 pixels); tiles straddle samples
    ("conv2", 3, 7, 9, False, None),
    # the model's shape: 81 rows per sample against 16-row tiles
    ("conv2", 5, 20, 20, False, None),
    # one output pixel
    ("conv3", 1, 3, 3, False, None),
    # 3x2 outputs, 18 rows over three samples
    ("conv3", 3, 5, 4, False, None),
    # the model's shape: two samples per group, ragged last group
    ("conv3", 5, 9, 9, False, None),
    # two persistent workgroups, 9 groups of 25 tiny images, the last
    # one ragged: each takes over a prefetched group at least three times
    ("conv2", 203, 4, 4, False, 2),
    # groups of 25 (forward) and 9 (data gradient), ragged last groups
    ("conv3", 203, 3, 3, False, 2),
    # the NCHW-flattened store, 6, 49 and 6 pixels per channel
    ("conv3", 3, 5, 4, True, None),
    ("conv3", 5, 9, 9, True, None),
    ("conv2", 3, 7, 9, True, None),
]


def case_id(case):
    geom, n, h, w, flat, wg = case
    return f"{geom}-{n}x{h}x{w}" + ("-flat" if flat else "") + (
        f"-wg{wg}" if wg else "")


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """bf16-representable float64 CPU tensors x [N,Cin,H,W], w, b and gy
    [N,Cout,OH,OW]; s = conv(x, w) + b in float64; and ``bound``, the
    elementwise bound on |y - relu(s)| (derived in test_conv_igemm_gpu).

    ``integer``: |x| <= 4, |w| <= 3, |b| <= 8, |gy| <= 4. The largest
    forward sum is 576 * 12 + 8 = 6920 and the largest data-gradient sum
    576 * 12 = 6912, far below 2^24: fp32 accumulation is exact in any
    order. ``normal``: x ~ N(0, 1), w ~ N(0, 1/K) so that the conv is
    about N(0, 1), b ~ N(-0.5, 1): over half of the outputs are clamped."""
    geom, n, h, w_, _, _ = case
    cin, cout, k, stride = GEOMETRY[geom]
    oh, ow = (h - k) // stride + 1, (w_ - k) // stride + 1
    shapes = ((n, cin, h, w_), (cout, cin, k, k), (cout,), (n, cout, oh, ow))
    g = t.Generator().manual_seed(1000 + CASES.index(case))
    if kind == "integer":
        vals = [t.randint(-r, r + 1, shape, generator=g)
                for r, shape in zip((4, 3, 8, 4), shapes)]
    else:
        vals = [t.randn(shape, generator=g) for shape in shapes]
        vals[1] /= (cin * k * k) ** 0.5
        vals[2] -= 0.5
    x, w, b, gy = (v.to(t.bfloat16).double() for v in vals)
    s = F.conv2d(x, w, b, stride)
    bound = (2.0 ** -8 * s.clamp_min(0.0)
             + cin * k * k * 2.0 ** -23 * F.conv2d(x.abs(), w.abs(), None,
                                                   stride))
    return SimpleNamespace(x=x, w=w, b=b, gy=gy, s=s, bound=bound,
                           stride=stride, k=k, cout=cout)


def backward_reference(case, kind, mask):
    """Float64 autograd of conv(x, w) + b for the upstream gradient gy
    where ``mask`` (the ReLU passes) and 0 elsewhere: dx, dW, db, and the
    sum of the magnitudes of dx's terms."""
    r = reference(case, kind)
    x, w, b = (v.clone().requires_grad_() for v in (r.x, r.w, r.b))
    g = t.where(mask, r.gy, 0.0)
    dx, dw, db = t.autograd.grad(F.conv2d(x, w, b, r.stride), (x, w, b), g)
    abs_sum = F.conv_transpose2d(
        g.abs(), r.w.abs(), None, r.stride, output_padding=tuple(
            x.shape[d] - (g.shape[d] - 1) * r.stride - r.k for d in (2, 3)))
    return dx, dw, db, abs_sum
